"""CPU test infrastructure: ``TrainingModule.training_step`` without and with a logger, dry, against the recording stand-in for
libstp3hip.so (tests/host_trace.py, tests/model_trace.py).

    STP3_TRACE_LOG=... STP3_REAL_LIB=.../libstp3hip.so python tests/visualisation_trace.py recorder.so

Driver of tests/test_visualisation_cpu.py.  After one warm-up step the log gets three marks: ``# plain`` before a step of the module as it is built
(no logger), ``# logged`` before a step with a stub logger attached and VIS_INTERVAL = 1, ``# videos <json>`` with what the
stub's ``add_video`` received."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def drive(recorder):
    import torch
    from tests import model_trace
    module, batch, _ = model_trace.dry_setup(recorder)
    log = open(os.environ['STP3_TRACE_LOG'], 'a')

    def mark(text):
        log.write(f'# {text}\n')
        log.flush()

    videos = []

    class Writer:
        def add_video(self, name, video, global_step=None, fps=None):
            videos.append({'name': name, 'shape': list(video.shape), 'dtype': str(video.dtype), 'global_step': global_step, 'fps': fps})

    module.model.prepare_plan(batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'], torch.device('cpu'))
    assert module.logger is None
    with torch.autocast('cpu', dtype=torch.bfloat16):          # (the first step also fills the caches of weight shadows)
        module.training_step(batch)
    mark('plain')
    with torch.autocast('cpu', dtype=torch.bfloat16):
        module.training_step(batch)
    module.logger = types.SimpleNamespace(experiment=Writer())
    module.cfg.VIS_INTERVAL = 1
    mark('logged')
    with torch.autocast('cpu', dtype=torch.bfloat16):
        module.training_step(batch)
    mark('videos ' + json.dumps(videos))


if __name__ == '__main__':
    drive(sys.argv[1])
