"""TEST INFRASTRUCTURE -- run the device entropy decode of the JPEG decoder (csrc/stp3_jpeg_huff.hip, with csrc/stp3_jpeg.hip
behind it) on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and store what came out.

    python tests/hipcpu/run_jpeg_huff.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_jpeg_huff_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Stored, per case of tests/jpeg_huff_cases.all_cases(): how many coefficient / table words of the device decode
differ from stp3_jpeg_entropy's, the status words, the decoded image, ``last_stats``; the same for multi_wg with
sync_rounds = 0; whether the guard regions around buffers of exactly the announced sizes survived; and, for every stream of
the corruption sweep and every crafted stream, how host mode and device mode ended."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import jpeg_cases as JC  # noqa: E402
from tests import jpeg_huff_cases as HC  # noqa: E402
from run_jpeg import setup  # noqa: E402

GUARD, POISON = 256, 0xA5


def guarded(nbytes):
    """A byte tensor of exactly `nbytes` between two poisoned guard regions: (the tensor, a check of the guards)."""
    whole = torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8)
    intact = lambda: bool((whole[:GUARD] == POISON).all() and (whole[GUARD + nbytes:] == POISON).all())
    return whole[GUARD:GUARD + nbytes], intact


def raw_device_decode(dec, data):
    """stp3_jpeg_scan_prepare and stp3_jpeg_entropy_device on one stream, every buffer of exactly its announced size between
    guards: (return code of prepare, status word or None, coefficients or None, tables, guards intact)."""
    from stp3_amd import _lib
    from stp3_amd.datas import JpegScanGroup, _geometry
    lib = _lib.lib()
    h = _lib.JpegHeader()
    if lib.stp3_jpeg_info(data, len(data), ctypes.byref(h)) != 0:
        return None
    stride = -(-lib.stp3_jpeg_scan_bytes(ctypes.byref(h), len(data)) // 4) * 4
    scan, ok_scan = guarded(stride)
    desc, ok_desc = guarded(ctypes.sizeof(_lib.JpegScanDesc))
    quant, ok_quant = guarded(384)
    exact = np.frombuffer(data, dtype=np.uint8).copy()                          # (a heap block of the stream's own length)
    rc = lib.stp3_jpeg_scan_prepare(exact.ctypes.data, len(data), scan.data_ptr(), stride, desc.data_ptr(), quant.data_ptr())
    intact = ok_scan() and ok_desc() and ok_quant()
    if rc != 0:
        return rc, None, None, None, intact
    words = desc.numpy().view(np.int32)
    grp = JpegScanGroup(_geometry(h), [0], stride, False)
    grp.max_subs, grp.max_segs = int(words[0]), int(words[1])
    coef, ok_coef = guarded(2 * h.coef_count)
    status, ok_status = guarded(4)
    d = _lib.JpegHuffDims(1, h.width, h.height, h.components, h.hs, h.vs, stride, grp.max_subs, grp.max_segs)
    nbytes = _lib.c_size_t()
    assert lib.stp3_jpeg_entropy_workspace_bytes(ctypes.byref(d), dec.sync_rounds, ctypes.byref(nbytes)) == 0
    work, ok_work = guarded(nbytes.value)
    dec.entropy_device_launch(grp, scan.view(1, stride), desc.view(1, -1), coef.view(torch.int16).view(1, -1), status.view(torch.int32),
                              workspace=work)
    intact = intact and ok_scan() and ok_desc() and ok_coef() and ok_status() and ok_work()
    return rc, int(status.view(torch.int32)[0]), coef.view(torch.int16).numpy().copy(), quant.view(torch.int16).numpy().copy(), intact


def ending(dec, stream):
    """How a call on one stream ends: ('ok', digest of the image) or ('raised', exception type, message)."""
    try:
        return ['ok', HC.digest(dec([stream], 'cpu').numpy())]
    except Exception as e:  # noqa: BLE001
        return ['raised', type(e).__name__, str(e)]


def sweep_streams(fixture):
    """name -> the streams of the corruption sweep: every truncation of wg_sync at a subsequence edge +- 1 byte and
    HC.CORRUPTIONS seeded single-byte corruptions of each stream of HC.SWEEP."""
    out = {}
    s = HC.streams(fixture, 'wg_sync')[0]
    first = HC.scan_offset(s)
    for edge in range(first + HC.S, len(s), HC.S):
        for cut in (edge - 1, edge, edge + 1):
            if cut < len(s):
                out[f'cut/{cut}'] = s[:cut]
    rng = np.random.RandomState(20240)
    for name in HC.SWEEP:
        s = HC.streams(fixture, name)[0]
        for k in range(HC.CORRUPTIONS):
            at, b = int(rng.randint(0, len(s))), bytearray(s)
            if k % 3 == 0:
                at = int(rng.randint(HC.scan_offset(s), len(s)))                # (a third of them surely in the scan)
            b[at] = (b[at] ^ (1 << int(rng.randint(0, 8)))) if k & 1 else int(rng.randint(0, 256))
            out[f'{name}/{k}@{at}'] = bytes(b)
    return out


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd import _lib
    from stp3_amd.datas import JpegDecoder
    fixtures = {'jpeg': JC.load(), 'huff': HC.load()}
    host, dev = JpegDecoder(workers=2), JpegDecoder(workers=2, entropy='device')
    assert host.entropy_mode == 'host'
    out, report = {}, {'stats': {}, 'guards': {}, 'status': {}, 'sweep': {}, 'crafted': {}}
    for key, name in HC.all_cases():
        streams = (JC if key == 'jpeg' else HC).streams(fixtures[key], name)
        want = host.entropy(streams)
        groups, batch = dev.entropy_device(streams, 'cpu')
        report['stats'][name + '/entropy'] = dev.last_stats
        assert [(g.geometry, g.indices) for g in groups] == want.layout()
        out[f'{name}/coef_differ'] = np.array(sum(int((g.coef != w.coef).sum()) for g, w in zip(groups, want.groups)))
        out[f'{name}/quant_differ'] = np.array(sum(int((g.quant != w.quant).sum()) for g, w in zip(groups, want.groups)))
        out[f'{name}/rgb'] = dev(streams, 'cpu').numpy()
        report['stats'][name] = dev.last_stats
        raws = [raw_device_decode(dev, s) for s in streams]
        report['guards'][name] = [bool(r[4]) for r in raws]
        report['status'][name] = [[r[0], r[1]] for r in raws]
        coefs = want.groups[0].coef.numpy()
        out[f'{name}/raw_differ'] = np.array(sum(int((r[2] != coefs[k]).sum()) for k, r in enumerate(raws)))
    # the cross-workgroup rounds switched off: not converged, the host decoder takes the image
    none = JpegDecoder(workers=2, entropy='device', sync_rounds=0)
    streams = HC.streams(fixtures['huff'], 'multi_wg')
    report['status']['multi_wg/rounds0'] = raw_device_decode(none, streams[0])[1]
    out['multi_wg/rounds0/rgb'] = none(streams, 'cpu').numpy()
    report['stats']['multi_wg/rounds0'] = none.last_stats
    report['status']['wg_sync/rounds0'] = raw_device_decode(none, HC.streams(fixtures['huff'], 'wg_sync')[0])[1]
    # the corruption sweep: device mode ends as host mode ends
    for name, s in sweep_streams(fixtures['huff']).items():
        a, b = ending(host, s), ending(dev, s)
        raw = raw_device_decode(dev, s)
        report['sweep'][name] = {'host': a, 'device': b, 'stats': dev.last_stats, 'guards': True if raw is None else bool(raw[4]),
                                 'status': None if raw is None else [raw[0], raw[1]]}
    for name, s in JC.crafted_refused().items():
        raw = raw_device_decode(dev, s)
        report['crafted'][name] = {'host': ending(host, s), 'device': ending(dev, s), 'status': [raw[0], raw[1]], 'guards': bool(raw[4])}
    report['codes'] = {'irregular': _lib.STP3_JPEG_IRREGULAR, 'not_converged': _lib.STP3_JPEG_NOT_CONVERGED, 'einval': _lib.STP3_EINVAL}
    out['report'] = np.array(json.dumps(report))
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
