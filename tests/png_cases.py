"""The cases of the PNG decoder's tests (tests/test_png_cpu.py, tests/test_png_gpu.py, tests/hipcpu/run_png.py): the smallest
shapes at which each mechanism of the scanline reconstruction can go wrong.

HANDMADE cases are built here, deterministically: a source array, a filter type per row, and a small PNG WRITER (for the tests
only) that filters forward -- the forward filter reads original neighbours only, so it is a few array statements -- and wraps
the result with zlib into IHDR / (PLTE) / IDAT(s) / IEND with correct CRCs.  PNG is lossless: the expected output of every
handmade case is its source array.  STORED cases (tests/golden/png_cases.npz, written by scripts/make_golden_png.py) hold
streams Pillow's own encoder wrote, the four streams of formats the decoder leaves to its fallback, and the sha256 of Pillow's
decode of every stored stream: a different Pillow on another machine cannot move the tests.  Every comparison of this feature is
exact equality of every byte."""
import hashlib
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'png_cases.npz')
BAND = 64                                            # rows a wave of the kernel owns at a time (csrc/stp3_png.hip)
PASS = 8 * BAND                                       # rows a workgroup of the kernel covers in one pass
COLOUR_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}        # grey, grey + alpha, RGB, RGBA
HOSTILE_BYTES = (0, 1, 2, 3, 4, 253, 254, 255)       # small clusters: every tie of the Paeth rule occurs, sums wrap
RUNS = [4, 4, 1, 4, 0, 2, 3, 1, 1, 4]

# name -> hw, channels (1: (H, W) grey), filters: 'random' | a list per row | one type for all rows; images > 1: several streams
# of one geometry for one launch; alphabet: the byte values the source is drawn from (default: all 256)
HANDMADE = {}
for _c in (1, 2, 3, 4):                              # x < bpp, row 0, one lane
    for _h, _w in ((1, 1), (1, 7), (9, 1)):
        HANDMADE[f'extreme_{_h}x{_w}_c{_c}'] = dict(hw=(_h, _w), channels=_c, filters='random')
HANDMADE.update({
    'paeth_first_5x3': dict(hw=(5, 3), channels=3, filters=[4, 3, 2, 1, 0]),          # every type against a zero row above
    'band_63x5': dict(hw=(63, 5), channels=3, filters='random'),                      # the skew is longer than the row
    'band_64x2': dict(hw=(64, 2), channels=3, filters='random'),
    'band_65x70': dict(hw=(65, 70), channels=3, filters='random'),                    # one row carried into a second band
    'band_130x33': dict(hw=(130, 33), channels=3, filters='random'),                  # three bands
    'pass_515x5': dict(hw=(515, 5), channels=3, filters='random'),                    # a second pass: the carry row in LDS
    'pass_580x70': dict(hw=(580, 70), channels=1, filters='random'),                  # ... whose second pass has two bands
    **{f'only_type_{t}': dict(hw=(40, 40), channels=3, filters=t) for t in range(5)},
    'hostile_paeth': dict(hw=(24, 48), channels=1, filters=4, alphabet=HOSTILE_BYTES),         # ties, a = b = c
    'hostile_paeth_rgb': dict(hw=(70, 9), channels=3, filters=4, alphabet=HOSTILE_BYTES),
    'hostile_average': dict(hw=(24, 48), channels=2, filters=3, alphabet=HOSTILE_BYTES),       # a + b >= 256, wrapping sums
    'independent_runs': dict(hw=(10, 12), channels=3, filters=RUNS),                  # rows that do not read the row above
    'carla_300x400': dict(hw=(300, 400), channels=3, filters='random'),               # the real geometry
    'rgba_70x33': dict(hw=(70, 33), channels=4, filters='random'),
    'grey_65x257': dict(hw=(65, 257), channels=1, filters='random'),                  # row pitch 258 = 2 mod 4
    'three_images': dict(hw=(20, 24), channels=3, filters='random', images=3),        # per-image addressing
    'three_images_replay': dict(hw=(20, 24), channels=3, filters='random', images=3, seed=50),
    'wide_2x16384': dict(hw=(2, 16384), channels=1, filters=[3, 4]),                  # the width limit: more than 64 KB of dynamic LDS
    'wide_3x16384_rgba': dict(hw=(3, 16384), channels=4, filters=[1, 4, 3]),
    'three_idat': dict(hw=(33, 21), channels=3, filters='random', idat=(17, 301)),    # chunk concatenation, odd offsets
})
# streams stored in the fixture: Pillow's encoder (what its save() gets) ...
PILLOW = {
    'pillow_rgb': dict(hw=(48, 64), mode='RGB', save={}),                             # adaptive filters
    'pillow_optimize': dict(hw=(48, 64), mode='RGB', save=dict(optimize=True)),
    'pillow_palette_trns': dict(hw=(31, 45), mode='P', save=dict(transparency=3)),    # PLTE + tRNS
    'pillow_phys_text': dict(hw=(20, 30), mode='L', save=dict(dpi=(72, 72)), text=True),       # pHYs + tEXt
    'pillow_large': dict(hw=(150, 152), mode='RGB', save={}, noise=True),             # more than one IDAT chunk
}
# ... and what the decoder leaves to its fallback (written by the helpers below, decoded by Pillow)
UNSUPPORTED = ('adam7_rgb', 'rgb_16bit', 'palette_4bit', 'grey_1bit', 'grey_alpha_16bit')   # (Pillow: 16-bit grey + alpha -> 8-bit RGBA)
# ... and what it refuses even with the fallback: Pillow's decode (mode I;16, uint16) does not fit the uint8 result
REFUSED = ('grey_16bit',)
SUPPORTED = list(HANDMADE) + list(PILLOW)
CORRUPT = ('idat_crc', 'truncated', 'one_scanline_short', 'filter_type_5', 'bad_signature', 'zlib_garbage')


# ---- sources ---------------------------------------------------------------------------------------------------------------
def _rng(name, k=0, seed=0):
    return np.random.RandomState((zlib.crc32(name.encode()) + seed + k) % (1 << 31))         # (a case's bytes depend on its name only)


def source(name, k=0):
    """The k-th source image of a handmade case: uniformly random bytes (of the case's alphabet), (H, W) or (H, W, C) uint8."""
    c = HANDMADE[name]
    h, w = c['hw']
    shape = (h, w) if c['channels'] == 1 else (h, w, c['channels'])
    rng = _rng(name, k, c.get('seed', 0))
    if 'alphabet' in c:
        return np.array(c['alphabet'], dtype=np.uint8)[rng.randint(0, len(c['alphabet']), size=shape)]
    return rng.randint(0, 256, size=shape).astype(np.uint8)


def filters(name, k=0):
    c = HANDMADE[name]
    f = c['filters']
    if isinstance(f, str):
        return [int(v) for v in _rng(name, k, 7 + c.get('seed', 0)).randint(0, 5, size=c['hw'][0])]
    return list(f) if isinstance(f, (list, tuple)) else [f] * c['hw'][0]


def photo(h, w, seed, channels=3):
    """Smooth gradients + a little noise + flat rectangles: content on which an adaptive encoder uses every filter type."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], axis=2)
    img = img + rng.randint(-6, 7, size=img.shape)
    for _ in range(4):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + 1 + h // 3, x0:x0 + 1 + w // 3] = rng.randint(0, 256, size=3)
    img = img.clip(0, 255).astype(np.uint8)
    return img if channels == 3 else img[:, :, 1].copy()


# ---- the writer (tests only) -----------------------------------------------------------------------------------------------
def filter_rows(img, row_filters):
    """Forward-filter an (H, W) / (H, W, C) uint8 image: (H, 1 + W * C) uint8 scanlines.  A type above 4 leaves the bytes
    as they are (what a corrupt stream would hold)."""
    h = img.shape[0]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    x = img.reshape(h, -1).astype(np.int32)
    a = np.concatenate([np.zeros((h, bpp), np.int32), x[:, :-bpp]], axis=1)
    b = np.concatenate([np.zeros((1, x.shape[1]), np.int32), x[:-1]], axis=0)
    c = np.concatenate([np.zeros((h, bpp), np.int32), b[:, :-bpp]], axis=1)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    ft = np.asarray(row_filters, dtype=np.int32).reshape(h, 1)
    pred = np.select([ft == 1, ft == 2, ft == 3, ft == 4], [a, b, (a + b) >> 1, paeth], 0)
    return np.concatenate([ft.astype(np.uint8), ((x - pred) & 255).astype(np.uint8)], axis=1)


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(body, zlib.crc32(kind)))


def wrap(width, height, depth, colour, scanlines, interlace=0, palette=None, idat=(), before_idat=b''):
    """A PNG file around raw scanline bytes; ``idat``: offsets at which the compressed data is cut into several IDAT chunks."""
    data = zlib.compress(bytes(scanlines), 6)
    cuts = [0] + [min(o, len(data)) for o in idat] + [len(data)]
    out = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, depth, colour, 0, 0, interlace))
    if palette is not None:
        out += chunk(b'PLTE', bytes(palette))
    out += before_idat
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out += chunk(b'IDAT', data[lo:hi])
    return out + chunk(b'IEND', b'')


def write_png(img, row_filters, idat=()):
    """An 8-bit, non-interlaced PNG of ``img`` with the given filter type per row."""
    channels = 1 if img.ndim == 2 else img.shape[2]
    return wrap(img.shape[1], img.shape[0], 8, COLOUR_OF_CHANNELS[channels], filter_rows(img, row_filters).tobytes(), idat=idat)


def handmade_streams(name):
    c = HANDMADE[name]
    return [write_png(source(name, k), filters(name, k), idat=c.get('idat', ())) for k in range(c.get('images', 1))]


def unsupported_stream(name):
    """The formats of the fallback (and the refused one), every scanline with filter type None."""
    rng = _rng(name)
    none = lambda rows: b''.join(b'\0' + bytes(r) for r in rows)
    if name == 'adam7_rgb':
        img, passes = rng.randint(0, 256, size=(11, 13, 3)).astype(np.uint8), b''
        for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
            sub = img[y0::dy, x0::dx]
            if sub.size:
                passes += none(r.tobytes() for r in sub)
        return wrap(13, 11, 8, 2, passes, interlace=1)
    if name == 'rgb_16bit':
        img = rng.randint(0, 65536, size=(6, 9, 3)).astype('>u2')
        return wrap(9, 6, 16, 2, none(r.tobytes() for r in img))
    if name == 'grey_alpha_16bit':
        img = rng.randint(0, 65536, size=(6, 9, 2)).astype('>u2')
        return wrap(9, 6, 16, 4, none(r.tobytes() for r in img))
    if name == 'grey_16bit':
        img = rng.randint(0, 65536, size=(6, 9)).astype('>u2')
        return wrap(9, 6, 16, 0, none(r.tobytes() for r in img))
    if name == 'palette_4bit':
        idx = rng.randint(0, 16, size=(7, 10)).astype(np.uint8)
        return wrap(10, 7, 4, 3, none(((r[0::2] << 4) | r[1::2]).tobytes() for r in idx), palette=rng.randint(0, 256, size=48).astype(np.uint8))
    if name == 'grey_1bit':
        bits = rng.randint(0, 2, size=(9, 21)).astype(np.uint8)
        return wrap(21, 9, 1, 0, none(np.packbits(r).tobytes() for r in bits))
    raise KeyError(name)


def corrupt(name):
    """A stream the decoder must refuse (and never hand to the kernel or to Pillow)."""
    img, ft = source('independent_runs'), filters('independent_runs')
    good = write_png(img, ft)
    at = good.index(b'IDAT')
    if name == 'idat_crc':
        end = at + 4 + struct.unpack_from('>I', good, at - 4)[0]
        return good[:end] + bytes([good[end] ^ 0x40]) + good[end + 1:]
    if name == 'truncated':
        return good[:at + 20]
    if name == 'one_scanline_short':
        return wrap(img.shape[1], img.shape[0], 8, 2, filter_rows(img, ft)[:-1].tobytes())
    if name == 'filter_type_5':
        return write_png(img, ft[:6] + [5] + ft[7:])
    if name == 'bad_signature':
        return b'\x89PNG\r\n\x1a\r' + good[8:]
    if name == 'zlib_garbage':
        body = bytes(np.random.RandomState(5).randint(0, 256, size=200).astype(np.uint8))
        return good[:at - 4] + chunk(b'IDAT', body) + chunk(b'IEND', b'')
    raise KeyError(name)


# ---- access ----------------------------------------------------------------------------------------------------------------
def load():
    """The stored fixture: '<case>/<k>/png' (uint8 bytes of the stream), '<case>/<k>/sha256' (of Pillow's decode, the bytes
    of ``np.asarray(Image.open(...))`` with a boolean image as 0 / 1) and '<case>/<k>/shape'."""
    return dict(np.load(GOLDEN))


def count(name):
    return HANDMADE.get(name, {}).get('images', 1)


def streams(fixture, name):
    if name in HANDMADE:
        return handmade_streams(name)
    return [fixture[f'{name}/{k}/png'].tobytes() for k in range(count(name))]


def expected(fixture, name):
    """The source arrays of a handmade case, stacked: (images, H, W[, C]); None for a stored case (see ``digest``)."""
    return np.stack([source(name, k) for k in range(count(name))]) if name in HANDMADE else None


def sha256(array):
    return hashlib.sha256(np.ascontiguousarray(array).astype(np.uint8).tobytes()).hexdigest()


def digest(fixture, name):
    """(shape, sha256) of the expected decode of every image of a case."""
    if name in HANDMADE:
        return [(source(name, k).shape, sha256(source(name, k))) for k in range(count(name))]
    return [(tuple(int(v) for v in fixture[f'{name}/{k}/shape']), str(fixture[f'{name}/{k}/sha256'])) for k in range(count(name))]


def matches(fixture, name, got):
    """Whether ``got`` -- an array (images, ...) or a list of arrays -- is the expected decode of the case, byte for byte."""
    want = digest(fixture, name)
    return len(got) == len(want) and all(tuple(g.shape) == shape and sha256(g) == sha for g, (shape, sha) in zip(got, want))


# ---- a CARLA sample as PNG files ---------------------------------------------------------------------------------------------
def carla_files(seed=0, t=2, s=4):
    """PNG bytes of one small synthetic sample, written by the test writer, and the arrays they hold: sources just above the
    256 and 200 windows (the top-down image: 224 x 226 -> 203 x 205 after the resize by 1.1)."""
    rng = np.random.RandomState(seed)
    ft = lambda h: [int(v) for v in rng.choice([0, 1, 2, 2, 1, 4, 3], size=h)]
    cams = rng.randint(0, 256, size=(t, 4, 258, 260, 3)).astype(np.uint8)
    deps = rng.randint(0, 256, size=(t, 4, 258, 260, 3)).astype(np.uint8)
    colours = np.array([(255, 0, 255), (54, 52, 46), (0, 0, 0), (255, 0, 254)], dtype=np.uint8)
    maps = colours[rng.randint(0, 4, size=(t, 203, 201))]
    tops = np.array([10, 4, 0, 7], dtype=np.uint8)[rng.randint(0, 4, size=(s, 224, 226))]
    files = dict(image_files=[[write_png(cams[i, j], ft(258)) for j in range(4)] for i in range(t)],
                 depth_files=[[write_png(deps[i, j], ft(258)) for j in range(4)] for i in range(t)],
                 hdmap_files=[write_png(maps[i], ft(203)) for i in range(t)],
                 topdown_files=[write_png(tops[i], ft(224)) for i in range(s)])
    poses = np.cumsum(rng.rand(3, s), axis=1)
    measurements = dict(seq_x=list(poses[0]), seq_y=list(poses[1]), seq_theta=list(poses[2] * 0.1), x_command=3.0, y_command=-2.0,
                        command=2, steer=0.05, throttle=0.4, brake=0.0, velocity=4.5, receptive_field=t, sample_num=10)
    return files, (cams, deps, maps, tops), measurements


def sample_difference(got, want):
    """The keys on which two sample dictionaries differ (tensors bit for bit)."""
    import torch
    bad = [k for k in set(got) | set(want) if k not in got or k not in want]
    for k in set(got) & set(want):
        a, b = got[k], want[k]
        if torch.is_tensor(a) != torch.is_tensor(b):
            bad.append(k)
        elif torch.is_tensor(a):
            if a.dtype != b.dtype or a.shape != b.shape or not torch.equal(a.cpu(), b.cpu()):
                bad.append(k)
        elif a != b:
            bad.append(k)
    return sorted(bad)
