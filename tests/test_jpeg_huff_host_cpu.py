"""CPU: stp3_jpeg_scan_prepare (csrc/stp3_jpeg_entropy.h), the host half of the device entropy decode, under AddressSanitizer
and UndefinedBehaviorSanitizer in a stand-alone program of its own (tests/jpeg_huff_host/main.cpp), built exactly as
tests/test_jpeg_sanitize_cpu.py builds its program: the host compiler, no HIP, no Python in the process, nothing preloaded.
Inputs: the fixture streams of both JPEG fixtures, every truncation of two of them, 4 000 seeded corruptions and the crafted
streams.  For the streams it accepts, the unstuffed bytes and the segment table are compared with tests/jpeg_huff_cases.walk,
the same walk stated in Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_cases as JC
from tests import jpeg_huff_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRUPTIONS = 4000
EUNSUP = -10002


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    tmp = tmp_path_factory.mktemp('jpeg_huff_host')
    exe = str(tmp / 'jpeg_huff_host')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'st-p3_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'jpeg_huff_host', 'main.cpp'), '-o', exe]
    probe = tmp / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    flags = None
    for extra in (['-static-libasan', '-static-libubsan'], []):
        p = subprocess.run([cxx, '-fsanitize=address,undefined', str(probe), '-o', str(tmp / 'probe')] + extra, capture_output=True, text=True, timeout=600)
        if p.returncode == 0 and subprocess.run([str(tmp / 'probe')], capture_output=True, timeout=60).returncode == 0:
            flags = extra
            break
    if flags is None:
        pytest.skip('the host compiler cannot build and run a trivial program with -fsanitize=address,undefined')
    out = subprocess.run(cmd + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return tmp, exe


def test_scan_prepare_is_clean_and_states_the_walk(program):
    tmp, exe = program
    fixtures = {'jpeg': JC.load(), 'huff': HC.load()}
    named = [(name, s) for name in JC.CASES for s in JC.streams(fixtures['jpeg'], name)]
    named += [(name, s) for name in HC.CASES for s in HC.streams(fixtures['huff'], name)]
    named += list(JC.crafted_refused().items())                                 # valid syntax: prepared, refused later by the decode
    # irregular by construction: fill bytes in front of EOI, a restart marker out of sequence, no EOI
    rst = HC.streams(fixtures['huff'], 'wg_sync_rst')[0]
    at = rst.index(b'\xff\xd1')
    irregular = [rst[:-2] + b'\xff\xff\xd9', rst[:at] + b'\xff\xd2' + rst[at + 2:], rst[:-2]]
    named += [('irregular', s) for s in irregular]
    names = [n for n, _ in named]
    path, result = str(tmp / 'streams.bin'), str(tmp / 'out.bin')
    with open(path, 'wb') as f:
        for _, s in named:
            f.write(struct.pack('<I', len(s)) + s)
    out = subprocess.run([exe, path, result, str(names.index('wg_sync_rst')), str(names.index(JC.TRUNCATE[0])), str(CORRUPTIONS)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert 'failures 0' in out.stdout and f'streams {len(named)} ' in out.stdout, out.stdout
    blob, pos = open(result, 'rb').read(), 0
    prepared = 0
    for name, s in named:
        rc, = struct.unpack_from('<i', blob, pos)
        pos += 4
        if name in JC.UNSUPPORTED:
            assert rc == EUNSUP, name
            continue
        if name == 'irregular':
            assert rc == 10011
            continue
        assert rc == 0, name
        prepared += 1
        nsub, nseg = struct.unpack_from('<ii', blob, pos)
        records = np.frombuffer(blob, dtype='<i4', count=3 * nseg, offset=pos + 8).reshape(nseg, 3)
        scan = blob[pos + 8 + 12 * nseg:pos + 8 + 12 * nseg + HC.S * nsub]
        subseg = np.frombuffer(blob, dtype='<i4', count=nsub, offset=pos + 8 + 12 * nseg + HC.S * nsub)
        pos += 8 + 12 * nseg + HC.S * nsub + 4 * nsub
        want_scan, want_segments = HC.walk(s)
        assert scan == want_scan, name
        assert [tuple(r[:2]) for r in records.tolist()] == want_segments, name
        firsts = [a for a, _ in want_segments] + [nsub]
        assert subseg.tolist() == [k for k in range(nseg) for _ in range(firsts[k + 1] - firsts[k])], name
    assert pos == len(blob) and f'prepared {prepared},' in out.stdout
