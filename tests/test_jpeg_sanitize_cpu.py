"""CPU: the host entropy decoder (csrc/stp3_jpeg_entropy.h) under AddressSanitizer and UndefinedBehaviorSanitizer, in a
stand-alone program of its own (tests/jpeg_host/main.cpp): the host compiler, no HIP, no Python in the process, nothing
preloaded.  The decoder parses untrusted bytes; the program feeds it the fixture streams, every truncation of two of them and
a few thousand seeded single-byte and single-bit corruptions, each from heap blocks of exactly the announced sizes."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import jpeg_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRUPTIONS = 4000


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    tmp = tmp_path_factory.mktemp('jpeg_host')
    exe = str(tmp / 'jpeg_host')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'st-p3_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'jpeg_host', 'main.cpp'), '-o', exe]
    # Whether the toolchain HAS the sanitizer runtimes is asked with a trivial program; only that answer may skip.  gcc links
    # the runtimes dynamically unless told otherwise; linked statically the program does not depend on the order in which the
    # loader brings libraries in.
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


def test_entropy_decoder_is_clean_under_asan_and_ubsan(program):
    tmp, exe = program
    g = JC.load()
    names = [n for n in JC.CASES]
    streams = [s for n in names for s in JC.streams(g, n)]
    first = {n: sum(JC.CASES[m].get('images', 1) for m in names[:names.index(n)]) for n in names}
    whole = len(streams)
    streams += list(JC.crafted_refused().values())                              # valid syntax, values no encoder writes
    path = str(tmp / 'streams.bin')
    with open(path, 'wb') as f:
        for s in streams:
            f.write(struct.pack('<I', len(s)) + s)
    out = subprocess.run([exe, path, str(first[JC.TRUNCATE[0]]), str(first[JC.TRUNCATE[1]]), str(CORRUPTIONS)], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    supported = sum(JC.CASES[n].get('images', 1) for n in JC.SUPPORTED)
    assert whole == sum(JC.CASES[n].get('images', 1) for n in names)
    assert f'streams {len(streams)} decoded {supported},' in out.stdout and 'failures 0' in out.stdout, out.stdout
