"""Writes tests/golden/visualisation.npz: the reference's ``visualise_output`` (stp3/utils/visualisation.py:208-322), unmodified
and loaded from the reference tree, on the cases of tests/visualisation_cases.py, for tests/test_visualisation_cpu.py /
test_visualisation_gpu.py.

    python scripts/make_golden_visualisation.py

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, scipy, matplotlib and torch.  The reference's seventh panel
(``plot_planning``: a matplotlib figure read back with ``canvas.tostring_rgb``, which matplotlib 3.10 removed) is replaced AT RUN
TIME by a zero panel; the file on disk is untouched and the planning row of the stored videos is zero.  The reference shows
sample 0 only: sample b of a case is obtained by handing it the batch from b on.

Per case ``<name>/``:
  labels/<key>, output/<key>   the inputs (integers as int16, floats as float32 with bfloat16-representable values)
  consistent                   int16 (B, T, H, W): the instance ids the reference's own post-processing gave (cases with the
                               instance head)
  video                        uint8 (samples, 1, T, 3, 7 H, 2 W)
  fragile_share                float64: the largest share of fragile bytes over the flow panels (visualisation_cases.compare)
``meta/palette`` (70, 3) and ``meta/jet`` (256, 3) uint8: ``generate_instance_colours`` and ``uint8(jet(i) * 255)`` as the
reference's process computed them.  The properties the fixture is meant to have are asserted below, the fragile share and the
agreement of this project's CPU route (under the comparison rule) included.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from oracle import ref_stubs  # noqa: E402
from tests import visualisation_cases as VC  # noqa: E402

OUT = VC.GOLDEN


def load_reference():
    import matplotlib
    matplotlib.use('Agg')
    ref_stubs.install()
    import stp3.utils.visualisation as ref
    return ref


def run_reference(ref, labels, output, cfg, sample, shape):
    """(video (1, T, 3, 7 H, 2 W), consistent ids of the sample (T, H, W) or None) of the reference on clones of the inputs."""
    labels = {k: v[sample:].clone() for k, v in labels.items()}
    output = {k: v[sample:].clone() for k, v in output.items()}
    seen = []
    post, planning = ref.predict_instance_segmentation_and_trajectories, ref.plot_planning

    def recording(*args, **kwargs):
        seen.append(post(*args, **kwargs))
        return seen[-1]
    ref.predict_instance_segmentation_and_trajectories = recording                   # (module globals, for this call only)
    ref.plot_planning = lambda hd_map, traj, cfg: np.zeros(shape + (3,), dtype=np.uint8)
    try:
        video = ref.visualise_output(labels, output, cfg)
    finally:
        ref.predict_instance_segmentation_and_trajectories, ref.plot_planning = post, planning
    return video, (seen[0][0] if seen else None)


def main():
    ref = load_reference()
    from stp3_amd import visualisation as V
    from stp3_amd.instance import predict_instance_segmentation_and_trajectories
    out = {'meta/palette': np.stack([ref.generate_instance_colours({i: i for i in range(70)})[i] for i in range(70)]).astype(np.uint8),
           'meta/jet': np.uint8(ref.DEFAULT_COLORMAP(np.arange(256))[:, :3] * 255)}
    assert np.array_equal(out['meta/palette'], V.INSTANCE_COLOURS) and np.array_equal(out['meta/jet'], V.JET_BYTES)
    for name, c in VC.CASES.items():
        labels, output = VC.build(name)
        cfg = VC.cfg_of(name)
        T, H, W = c['T'], c['H'], c['W']
        before = {k: v.clone() for k, v in {**labels, **output}.items()}
        videos, consistent = [], []
        for sample in c['samples']:
            video, ids = run_reference(ref, labels, output, cfg, sample, (H, W))
            assert video.shape == (1, T, 3, 7 * H, 2 * W) and video.dtype == np.uint8
            assert not video[0, :, :, 6 * H:].any(), 'the planning row of the stored video is zero'
            videos.append(video)
            consistent.append(ids)
        assert all(torch.equal(v, before[k]) for k, v in {**labels, **output}.items())
        pre = f'{name}/'
        for group, tensors in (('labels', labels), ('output', output)):
            for k, v in tensors.items():
                assert v.is_floating_point() or int(v.abs().max()) < 32768
                if v.is_floating_point() and 'traj' not in k:
                    assert torch.equal(v, v.bfloat16().float()), f'{name}/{k} is not representable in bfloat16'
                out[f'{pre}{group}/{k}'] = v.numpy().astype(np.float32 if v.is_floating_point() else np.int16)
        out[pre + 'video'] = np.stack(videos)
        if c['instance']:
            assert c['samples'] == tuple(range(c['B']))
            out[pre + 'consistent'] = torch.stack(consistent).numpy().astype(np.int16)
            mine = predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False)
            assert np.array_equal(mine.numpy(), out[pre + 'consistent']), f'{name}: this project numbers the instances differently'
    np.savez_compressed(OUT, **out)
    VC.fixture.cache_clear()
    for name, c in VC.CASES.items():                                                   # from the file, as the tests see it
        labels, output, consistent = VC.stored(name)
        built = VC.build(name)
        assert all(torch.equal(v, built[0][k]) for k, v in labels.items()) and all(torch.equal(v, built[1][k]) for k, v in output.items())
        share = 0.0
        for sample in c['samples']:
            mine = V.visualise_output_reference(labels, output, VC.cfg_of(name), sample=sample)
            share = max(share, VC.compare(name, mine.numpy(), sample, labels, output, 'CPU route'))
            for (row, side), x in VC.flow_sources(labels, output, sample, c['instance'], c['flow']).items():
                rad = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
                assert (rad[rad > 0] < 1).any() and (rad > 1).any(), f'{name}: {row} {side} has no vectors on both sides of 1'
        out[f'{name}/fragile_share'] = np.array(share)
        print(f'{name}: video {out[name + "/video"].shape}, fragile share of the flow panels at most {share:.3%}')
    full = VC.CASES['full']
    lab = out['full/labels/instance']
    assert full['H'] != full['W'] and full['W'] % 4 != 0 and 74 in lab and not (lab[0, 2] == 0).any() and lab[0, 2].min() == 1
    assert np.ptp(out['full/labels/centerness'][0, 1]) == 0
    assert VC.CASES['t1']['T'] == 1 and VC.CASES['t1']['W'] % 2 == 1
    assert not any(k.startswith('off/') and k.split('/')[-1] in ('instance', 'flow', 'pedestrian', 'instance_flow') for k in out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == '__main__':
    main()
