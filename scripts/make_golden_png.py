"""Writes tests/golden/png_cases.npz: the streams Pillow's own encoder writes for the PILLOW cases of tests/png_cases.py, the
four streams of formats the decoder leaves to its fallback, and for every stored stream the shape and the sha256 of Pillow's
decode -- the oracle of the PNG decoder's tests next to the handmade cases, whose oracle is their source array.

    python scripts/make_golden_png.py

Needs Pillow (the streams, once stored, are never re-encoded by a test)."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_cases as PC  # noqa: E402


def chunk_names(data):
    pos, names = 8, []
    while pos < len(data):
        names.append(data[pos + 4:pos + 8].decode())
        pos += 12 + int.from_bytes(data[pos:pos + 4], 'big')
    return names


def pillow_stream(name):
    from PIL import Image, PngImagePlugin
    c = PC.PILLOW[name]
    h, w = c['hw']
    seed = 3000 + sorted(PC.PILLOW).index(name)
    if c.get('noise'):
        src = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    else:
        src = PC.photo(h, w, seed, channels=1 if c['mode'] in ('L', 'P') else 3)
    if c['mode'] == 'P':
        im = Image.frombytes('P', (w, h), src.tobytes())                         # 256 entries: 8-bit indices
        im.putpalette([int(v) for v in np.random.RandomState(seed).randint(0, 256, size=768)])
    else:
        im = Image.fromarray(src)
    assert im.mode == c['mode'], (name, im.mode)
    save = dict(c['save'])
    if c.get('text'):
        text = PngImagePlugin.PngInfo()
        text.add_text('Title', 'a test vector')
        save['pnginfo'] = text
    buf = io.BytesIO()
    im.save(buf, 'PNG', **save)
    return buf.getvalue()


def main():
    import PIL
    from PIL import Image
    out = {}
    for name in list(PC.PILLOW) + list(PC.UNSUPPORTED):
        data = pillow_stream(name) if name in PC.PILLOW else PC.unsupported_stream(name)
        im = Image.open(io.BytesIO(data))
        decoded = np.asarray(im)
        out[f'{name}/0/png'] = np.frombuffer(data, dtype=np.uint8)
        out[f'{name}/0/shape'] = np.array(decoded.shape, dtype=np.int64)
        out[f'{name}/0/sha256'] = np.array(PC.sha256(decoded))
        print(f'{name}: {len(data)} bytes, mode {im.mode}, {decoded.dtype}{decoded.shape}, chunks {" ".join(chunk_names(data))}')
    out['meta'] = np.array(f'Pillow {PIL.__version__}')
    np.savez_compressed(PC.GOLDEN, **out)
    print(PC.GOLDEN, os.path.getsize(PC.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
