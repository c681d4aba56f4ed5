"""CPU test infrastructure: dry run of the EVAL forward through the GPU code path, without a GPU.

Driver of tests/test_inference_cpu.py (which holds the checks), on the recording stand-in of tests/host_trace.py and the
process patches of tests/model_trace.py.  Values are meaningless (the kernels do nothing); what the run establishes is WHICH
C-ABI calls the eval forward makes -- plainly (``model.eval()(...)``, the path the inference engine is pinned against) and
inside the engine's fused-eval scope (``stp3_amd.layers.fused.eval_fusion``: what ``InferenceEngine`` captures).

    STP3_TRACE_LOG=... STP3_REAL_LIB=.../libstp3hip.so python tests/inference_trace.py recorder.so plain|engine

The log is split by ``# encoder`` / ``# decoder`` / ``# full`` marks: the image encoder alone, the BEV decoder alone, the
whole Perception.yml forward.
"""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def drive(recorder, mode):
    import torch
    from tests import model_trace
    module, batch, _ = model_trace.dry_setup(recorder, full_losses=False)
    module.eval()
    model = module.model
    log = open(os.environ['STP3_TRACE_LOG'], 'a')

    def mark(text):
        log.write(f'# {text}\n')
        log.flush()

    if mode == 'engine':
        from stp3_amd import inference
        coefs = inference.EvalCoefficients(model, torch.device('cpu'))

        def scope():
            return coefs.scope()
    else:
        def scope():
            return contextlib.nullcontext()

    rf = model.receptive_field
    image = batch['image'][:, :rf]
    b, s, n, c, h, w = image.shape
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        mark('encoder')
        with scope():
            model.encoder(image.reshape(b * s * n, c, h, w))
        mark('decoder')
        x, y = model.bev_dimension[0].item(), model.bev_dimension[1].item()
        states = torch.zeros(b, rf, model.future_pred_in_channels, x, y, dtype=torch.bfloat16)
        with scope():
            model.decoder(states)
        mark('full')
        model.prepare_plan(batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'], torch.device('cpu'))
        with scope():
            out = model(batch['image'], batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'])
        model.prebuilt_plan = None
        mark('outputs ' + ' '.join(sorted(k for k, v in out.items() if v is not None)))
    mark('end')


if __name__ == '__main__':
    drive(sys.argv[1], sys.argv[2])
