"""CPU test infrastructure: dry run of ONE TICK of the streaming inference engine through the GPU code path, without a GPU.

Driver of tests/test_streaming_cpu.py (which holds the checks), on the recording stand-in of tests/host_trace.py and the process
patches of tests/model_trace.py, modelled on tests/inference_trace.py (whose model, batch and fused-eval scope it takes).  Values
are meaningless (the kernels do nothing); what the run establishes is WHICH C-ABI calls a tick makes:
``stp3_amd.inference.streaming_tick`` -- the function ``StreamingEngine`` captures -- inside the engine's fused-eval scope.

    STP3_TRACE_LOG=... STP3_REAL_LIB=.../libstp3hip.so python tests/streaming_trace.py recorder.so

The log is split by marks: ``# encoder`` -- the image encoder on the B * N newest images alone; ``# tick`` -- the whole tick;
``# shapes B T N`` and ``# outputs ...`` carry what the checks need besides.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def drive(recorder):
    import torch
    from tests import model_trace
    module, batch, _ = model_trace.dry_setup(recorder, full_losses=False)
    module.eval()
    model = module.model
    log = open(os.environ['STP3_TRACE_LOG'], 'a')

    def mark(text):
        log.write(f'# {text}\n')
        log.flush()

    from stp3_amd import inference
    coefs = inference.EvalCoefficients(model, torch.device('cpu'))
    rf = model.receptive_field
    b, _, n, c, h, w = batch['image'].shape
    newest = batch['image'][:, rf - 1].contiguous()
    mark(f'shapes {b} {rf} {n}')
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        mark('encoder')
        with coefs.scope():
            model.encoder(newest.reshape(b * n, c, h, w))
        mark('plan')
        plan = model.prepare_plan(batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'], torch.device('cpu'))
        model.prebuilt_plan = None
        d = plan.dims
        feat_window = torch.zeros(b, rf, d.NPIX, d.C)
        logits_window = torch.zeros(b, rf, d.NPIX, d.D)
        ego = batch['future_egomotion'].float()
        mark('tick')
        with coefs.scope():
            out = inference.streaming_tick(model, newest, feat_window, logits_window, plan, ego)
        mark('outputs ' + ' '.join(sorted(k for k, v in out.items() if v is not None)))
        mark('depth_prediction ' + ' '.join(str(s) for s in out['depth_prediction'].shape))
    mark('end')


if __name__ == '__main__':
    drive(sys.argv[1])
