"""TEST INFRASTRUCTURE -- run the loss / label-warp cases of csrc/stp3_loss.hip (tests/loss_cases.py) on CPU tensors through
libstp3hip_cpu.so (tests/hipcpu/build.py) and print the figures as JSON; ``abi`` instead of case names prints the return codes
of the C ABI's argument checks.

    python tests/hipcpu/run_loss.py <libstp3hip_cpu.so> [--repeat] <case name> [<case name> ...]
    python tests/hipcpu/run_loss.py <libstp3hip_cpu.so> abi

Driver of tests/test_loss_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  ``--repeat`` runs every operator twice and compares the bits (tests/loss_cases.REPEAT; off otherwise: the second pass
doubles the time of a case)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import torch  # noqa: E402

from tests import loss_cases as LC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_conv_pre.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def abi():
    """Return codes of the entry points for arguments they must reject -- every call returns before it launches anything."""
    from stp3_amd import _lib
    lib = _lib.lib()
    rows, c, p = 2, 2, 8
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)           # noqa: E731
    z, y, px, sel, out, g, dz = f32(rows, c, p), torch.zeros(rows, p, dtype=torch.int64), f32(rows, p), f32(rows, 2), f32(2), f32(1), f32(rows, c, p)
    ws = torch.zeros(1 << 14, dtype=torch.uint8)
    need = ctypes.c_size_t()

    def dims(r=rows, pp=p, dtype=_lib.DTYPE_F32):
        return _lib.CeDims(r, pp, c, 2, 255, dtype, c * pp, pp, 1)

    def fwd(d, logits=z, labels=y, loss=px, s=sel, o=out, w=ws, nbytes=None):
        dp = ctypes.byref(d) if d is not None else None
        ptr = [t.data_ptr() if t is not None else None for t in (logits, labels, loss, s, o, w)]
        return lib.stp3_ce_topk_fwd(dp, ptr[0], ptr[1], None, None, ptr[2], ptr[3], 1.0, 0, ptr[4], ptr[5],
                                    ws.numel() if nbytes is None else nbytes, 0)

    def bwd(d, logits=z, labels=y, loss=px, s=sel, gout=g, dl=dz):
        dp = ctypes.byref(d) if d is not None else None
        ptr = [t.data_ptr() if t is not None else None for t in (logits, labels, loss, s, gout, dl)]
        return lib.stp3_ce_topk_bwd(dp, ptr[0], ptr[1], None, None, ptr[2], ptr[3], ptr[4], 1.0, ptr[5], 0)
    res = {'ce_ws_null_dims': lib.stp3_ce_topk_workspace_bytes(None, ctypes.byref(need)),
           'ce_ws_null_bytes': lib.stp3_ce_topk_workspace_bytes(ctypes.byref(dims()), None),
           'ce_ws_rows0': lib.stp3_ce_topk_workspace_bytes(ctypes.byref(dims(r=0)), ctypes.byref(need)),
           'ce_fwd_null_dims': fwd(None), 'ce_fwd_rows0': fwd(dims(r=0)), 'ce_fwd_rows_neg': fwd(dims(r=-3)),
           'ce_fwd_null_logits': fwd(dims(), logits=None), 'ce_fwd_null_labels': fwd(dims(), labels=None),
           'ce_fwd_null_loss': fwd(dims(), loss=None), 'ce_fwd_null_sel': fwd(dims(), s=None), 'ce_fwd_null_out': fwd(dims(), o=None),
           'ce_fwd_null_ws': fwd(dims(), w=None), 'ce_fwd_dtype': fwd(dims(dtype=7)),
           'ce_fwd_short_ws': fwd(dims(), nbytes=rows * 8 - 1), 'ce_fwd_2g': fwd(dims(r=1 << 16, pp=1 << 15)),
           'ce_bwd_null_dims': bwd(None), 'ce_bwd_rows0': bwd(dims(r=0)), 'ce_bwd_null_logits': bwd(dims(), logits=None),
           'ce_bwd_null_gout': bwd(dims(), gout=None), 'ce_bwd_null_dlogits': bwd(dims(), dl=None), 'ce_bwd_dtype': bwd(dims(dtype=7)),
           'ce_bwd_2g': bwd(dims(r=1 << 16, pp=1 << 15))}
    pred, tgt, stat = f32(rows, c, p), f32(rows, c, p), f32(2)

    def rfwd(r=rows, norm=1, dtype=_lib.DTYPE_F32, x=pred, t=tgt, o=out, w=ws, nbytes=None):
        ptr = [v.data_ptr() if v is not None else None for v in (x, t, o, w)]
        return lib.stp3_reg_loss_fwd(r, c, p, norm, 255.0, dtype, ptr[0], ptr[1], None, ptr[2], ptr[3],
                                     ws.numel() if nbytes is None else nbytes, 0)

    def rbwd(r=rows, norm=1, dtype=_lib.DTYPE_F32, x=pred, t=tgt, st=stat, gout=g, dx=dz):
        ptr = [v.data_ptr() if v is not None else None for v in (x, t, st, gout, dx)]
        return lib.stp3_reg_loss_bwd(r, c, p, norm, 255.0, dtype, ptr[0], ptr[1], None, ptr[2], ptr[3], ptr[4], 0)
    _lib.check(lib.stp3_reg_loss_workspace_bytes(ctypes.byref(need)), 'stp3_reg_loss_workspace_bytes')
    res.update({'reg_ws_null': lib.stp3_reg_loss_workspace_bytes(None), 'reg_fwd_rows0': rfwd(r=0), 'reg_fwd_norm3': rfwd(norm=3),
                'reg_fwd_null_pred': rfwd(x=None), 'reg_fwd_null_target': rfwd(t=None), 'reg_fwd_null_out': rfwd(o=None),
                'reg_fwd_null_ws': rfwd(w=None), 'reg_fwd_dtype': rfwd(dtype=7), 'reg_fwd_short_ws': rfwd(nbytes=need.value - 1),
                'reg_bwd_rows0': rbwd(r=0), 'reg_bwd_norm3': rbwd(norm=3), 'reg_bwd_null_pred': rbwd(x=None),
                'reg_bwd_null_stat': rbwd(st=None), 'reg_bwd_null_gout': rbwd(gout=None), 'reg_bwd_null_dpred': rbwd(dx=None),
                'reg_bwd_dtype': rbwd(dtype=7)})
    x, th, yy = f32(1, 1, 4, 4), f32(6), f32(1, 1, 4, 4)

    def warp(fr=1, h=4, w=4, xx=x, t=th, o=yy):
        ptr = [v.data_ptr() if v is not None else None for v in (xx, t, o)]
        return lib.stp3_warp_nearest(fr, 1, h, w, ptr[0], ptr[1], None, ptr[2], 0)
    res.update({'warp_frames0': warp(fr=0), 'warp_null_x': warp(xx=None), 'warp_null_theta': warp(t=None), 'warp_null_y': warp(o=None),
                'warp_2g': warp(fr=2, h=1 << 15, w=1 << 15)})
    return res


def main(lib_path, names):
    ops = setup(lib_path)
    LC.REPEAT = '--repeat' in names
    names = [n for n in names if n != '--repeat']
    t0 = time.time()
    if names == ['abi']:
        res = abi()
    else:
        cases = dict(LC.case_list())
        res = {name: LC.run_case(ops, 'cpu', **cases[name]) for name in names}
    res['seconds'] = round(time.time() - t0, 1)
    print('RESULT', json.dumps(res))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2:])
