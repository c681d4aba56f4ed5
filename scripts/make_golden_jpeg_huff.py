"""Writes tests/golden/jpeg_huff_cases.npz: for every case of tests/jpeg_huff_cases.py the JPEG stream Pillow encodes from the
case's source image and the sha256 of the RGB bytes Pillow decodes from it (the pixels themselves stay out: the file holds
streams of a hundred kilobytes).

    python scripts/make_golden_jpeg_huff.py

`stuff_edge` is searched: the first seed whose stream has a stuffed FF 00 pair across a subsequence edge of the stuffed scan
and an FF as the last byte of a subsequence of the unstuffed one."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

from tests import jpeg_huff_cases as HC  # noqa: E402


def encode(src, save):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(src, 'RGB').save(buf, 'JPEG', **save)
    return buf.getvalue()


def main():
    import PIL
    from PIL import Image, features
    out = {}
    for name, c in HC.CASES.items():
        for k in range(c.get('images', 1)):
            save = c['save'][k] if isinstance(c['save'], list) else c['save']
            if c.get('search'):
                for seed in range(100000, 104000):
                    data = encode(HC.source(name, k, seed=seed), save)
                    if HC.stuffing_at_an_edge(data) == (True, True):
                        print(f'{name}: seed {seed}')
                        break
                else:
                    raise SystemExit(f'{name}: no seed found')
            else:
                data = encode(HC.source(name, k), save)
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
            assert rgb.shape == tuple(c['hw']) + (3,), (name, rgb.shape)
            out[f'{name}/{k}/jpeg'] = np.frombuffer(data, dtype=np.uint8)
            out[f'{name}/{k}/sha256'] = np.frombuffer(bytes.fromhex(HC.digest(rgb)), dtype=np.uint8)
            plain, segments = HC.walk(data)
            print(f'{name}/{k}: {len(data)} bytes, {len(plain) // HC.S} subsequences, {len(segments)} segments')
    out['meta'] = np.array(f'Pillow {PIL.__version__}, libjpeg-turbo {features.version("jpg")}, S {HC.S}, G {HC.G}')
    np.savez_compressed(HC.GOLDEN, **out)
    print(HC.GOLDEN, os.path.getsize(HC.GOLDEN), 'bytes')
    HC.load()


if __name__ == '__main__':
    main()
