"""TEST INFRASTRUCTURE -- run the depthwise cases of csrc/stp3_dwconv.hip (tests/dwconv_cases.py) on CPU tensors through
libstp3hip_cpu.so (tests/hipcpu/build.py) and print the figures as JSON; ``abi`` instead of case names prints the return codes
of the C ABI's argument checks next to the expected ones.

    python tests/hipcpu/run_dwconv.py <libstp3hip_cpu.so> <case name> [<case name> ...]
    python tests/hipcpu/run_dwconv.py <libstp3hip_cpu.so> abi

Driver of tests/test_dwconv_exact_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

from tests import dwconv_cases as DC  # noqa: E402


def main(lib_path, names):
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    lib = _lib.lib()
    t0 = time.time()
    if names == ['abi']:
        res = {'abi': DC.abi(lib, 'cpu')}
    else:
        cases = dict(DC.case_list())
        res = {}
        for name in names:
            t1 = time.time()
            res[name] = DC.run_case(lib, 'cpu', lambda: None, **cases[name])
            res[name]['seconds'] = round(time.time() - t1, 1)
    res['seconds'] = round(time.time() - t0, 1)
    print('RESULT', json.dumps(res))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2:])
