"""Writes tests/golden/jpeg_cases.npz: for every case of tests/jpeg_cases.py the JPEG byte stream Pillow encodes from the
case's source image and the RGB bytes Pillow decodes from that stream -- the oracle of the JPEG decoder's tests.

    python scripts/make_golden_jpeg.py

Needs Pillow linked against libjpeg-turbo (the streams, once stored, are never re-encoded by a test)."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_cases as JC  # noqa: E402


def segments(data):
    """(marker, payload) of every segment in front of the scan."""
    pos = 2
    while data[pos + 1] != 0xDA:
        n = (data[pos + 2] << 8) | data[pos + 3]
        yield data[pos + 1], data[pos + 4:pos + 2 + n]
        pos += 2 + n


def stream_411(template, h, w, seed):
    """A baseline stream with luma sampling 4x1 (4:1:1), which Pillow cannot write: the DQT and DHT segments of a Pillow
    stream verbatim, a frame and scan header of our own, and blocks that hold a DC coefficient only (flat 8 x 8 blocks)."""
    codes, keep = {}, b''
    for m, payload in segments(template):
        if m in (0xDB, 0xC4, 0xE0):
            keep += bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, 'big') + payload
        i = 0
        while m == 0xC4 and i < len(payload):
            counts, code, k = payload[i + 1:i + 17], 0, i + 17
            for length, cnt in enumerate(counts, 1):
                for _ in range(cnt):
                    codes[payload[i], payload[k]] = (code, length)
                    code, k = code + 1, k + 1
                code <<= 1
            i = k
    sof = bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, 0x41, 0, 2, 0x11, 1, 3, 0x11, 1])
    sos = bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    rng, bits, pred = np.random.RandomState(seed), [], [0, 0, 0]
    for _ in range(-(-h // 8) * -(-w // 32)):
        for comp, table in ((0, 0), (0, 0), (0, 0), (0, 0), (1, 1), (2, 1)):
            dc = int(rng.randint(-150, 151))
            diff, pred[comp] = dc - pred[comp], dc
            size = abs(diff).bit_length()
            code, length = codes[table, size]                               # class 0 (DC), table id: the high nibble is 0
            bits.append(format(code, f'0{length}b') + (format(diff if diff > 0 else diff + (1 << size) - 1, f'0{size}b') if size else ''))
            code, length = codes[0x10 | table, 0x00]                        # end of block
            bits.append(format(code, f'0{length}b'))
    bits = ''.join(bits)
    bits += '1' * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')
    return (b'\xff\xd8' + keep + b'\xff\xc0' + (len(sof) + 2).to_bytes(2, 'big') + sof +
            b'\xff\xda' + (len(sos) + 2).to_bytes(2, 'big') + sos + scan + b'\xff\xd9')


def main():
    import PIL
    from PIL import Image, features
    out = {}
    for name, c in JC.CASES.items():
        n = c.get('images', 1)
        for k in range(n):
            save = c['save'][k] if isinstance(c['save'], list) else c['save']
            src = JC.source(name, k)
            mode = 'L' if c.get('grey') else 'CMYK' if c.get('cmyk') else 'RGB'
            buf = io.BytesIO()
            Image.fromarray(src, mode).save(buf, 'JPEG', **save)
            data = buf.getvalue()
            if c.get('handmade_411'):
                data = stream_411(data, src.shape[0], src.shape[1], 411)
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
            assert rgb.shape == tuple(c['hw']) + (3,), (name, rgb.shape)
            out[f'{name}/{k}/jpeg'] = np.frombuffer(data, dtype=np.uint8)
            out[f'{name}/{k}/rgb'] = rgb
            print(f'{name}/{k}: {len(data)} bytes, layer {getattr(Image.open(io.BytesIO(data)), "layer", None)}')
    out['meta'] = np.array(f'Pillow {PIL.__version__}, libjpeg-turbo {features.version("jpg")}')
    np.savez_compressed(JC.GOLDEN, **out)
    print(JC.GOLDEN, os.path.getsize(JC.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
