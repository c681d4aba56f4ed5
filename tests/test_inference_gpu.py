"""GPU: ``stp3_amd.inference.InferenceEngine`` -- the eval forward as one hipGraph of fused kernels -- against the plain
``model.eval()(...)`` forward it is pinned to.

BIT-EQUALITY.  The fused eval operators keep the rounding points of the two operators they replace (include/stp3_hip.h:
stp3_conv2d_fwd_affine), so every non-None entry of the output dict must have the bit pattern of the plain forward under the
same autocast: Perception.yml at B = 4, T = 3 (the model and batch of tests/test_iou_gpu.py) and at B = 1, a
Prediction.yml-shaped model at the size tests/test_prediction_gpu.py uses, and a float32 engine (plain operators captured).
REPLAY: ten replays on one batch are bit-identical; a replay on a second batch (other poses, other images) equals the plain
forward on that batch (the plan and the ego-motion vector are rebuilt in place); after ``load_state_dict`` of perturbed weights
and running statistics the engine is STALE until ``refresh()`` (the shadows and the coefficient arena are what the graph
reads), and equal again after it -- on the Perception engine and on the Prediction-shaped one (whose GRU cells read merged gate
weights the engine owns); the example image is copied, never written.
REFERENCE PIN: the engine's bf16 Perception outputs meet the bounds of tests/test_iou_gpu.py on tests/golden/iou_b4.npz --
synthetic-label IoU within 1e-3, pseudo-label IoU within 2e-2, at most 1 pixel in 1 000 with another arg-max
(profiles/r04a_iou.json; not re-tuned).
ERRORS: a wrong shape, a model in training mode and a model on the CPU raise ``Stp3HipError``."""
import numpy as np
import pytest
import torch

from stp3_amd import synthetic
from stp3_amd.config import perception_cfg
from tests import helpers as H

pytestmark = pytest.mark.gpu
POSES = ('intrinsics', 'extrinsics', 'future_egomotion')


def _inputs(batch):
    return batch['image'].cuda(), batch['intrinsics'], batch['extrinsics'], batch['future_egomotion']


@torch.no_grad()
def _plain(model, batch, dtype=torch.bfloat16):
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype is not None):
        out = model(*_inputs(batch))
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def _mismatches(a, b):
    """{key: elements whose bit patterns differ} over the non-None entries (shape / dtype / key differences count as all)."""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    bad = {}
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
            bad[k] = -1
            continue
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a[k].element_size()]
        n = int((a[k].contiguous().view(view) != b[k].contiguous().view(view)).sum().item())
        if n:
            bad[k] = n
    return bad


def _perception_model():
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    g = H.load('iou_b4.npz')
    shifts = {k: float(g[f'shift/{k}'][0]) for k in H.IOU_HEADS}
    model = H.fill_deterministic(STP3(perception_cfg())).eval()
    H.prepare_heads(model.decoder, shifts, {k: bool(int(g[f'swap/{k}'][0])) for k in H.IOU_HEADS})
    return to_channels_last(model.cuda())


@pytest.fixture(scope='module')
def perception():
    """(model, batch, engine, engine outputs, plain outputs) of Perception.yml at B = 4, T = 3: the model and batch of
    tests/test_iou_gpu.py."""
    from stp3_amd.inference import InferenceEngine
    model = _perception_model()
    batch = synthetic.make_batch(batch=4, seq=3, seed=7)
    plain = _plain(model, batch)
    engine = InferenceEngine(model, batch, autocast_dtype=torch.bfloat16)
    out = engine(*_inputs(batch), clone=True)
    return model, batch, engine, out, plain


def test_perception_b4_bit_equal(perception):
    model, batch, engine, out, plain = perception
    bad = _mismatches(out, plain)
    print('[inference] Perception B=4: entries', sorted(k for k, v in out.items() if v is not None), 'mismatching elements', bad)
    assert not bad, bad
    assert engine.coefs is not None and len(engine.coefs.layers) > 100


def test_ten_replays_identical_and_static_outputs(perception):
    model, batch, engine, out, plain = perception
    image = engine.image                               # the static buffer handed back: no copy
    for i in range(10):
        again = engine(image, *[batch[k] for k in POSES])
        bad = _mismatches(again, out)
        assert not bad, (i, bad)
    assert all(again[k] is engine.outputs[k] for k in again)           # the static tensors, overwritten by the next call


def test_second_batch_rebuilds_plan_in_place(perception):
    model, batch, engine, out, plain = perception
    other = synthetic.make_batch(batch=4, seq=3, seed=11)
    assert not torch.equal(other['extrinsics'], batch['extrinsics']) and not torch.equal(other['image'], batch['image'])
    got = engine(*_inputs(other), clone=True)
    want = _plain(model, other)
    bad = _mismatches(got, want)
    print('[inference] second batch: mismatching elements', bad, '; differs from the first batch in',
          sorted(_mismatches(got, out)))
    assert not bad, bad
    assert _mismatches(got, out), 'the second batch gave the outputs of the first'
    back = engine(*_inputs(batch), clone=True)
    assert not _mismatches(back, out)


def test_reference_iou_bounds_through_the_engine(perception):
    from stp3_amd.metrics import IntersectionOverUnion
    model, batch, engine, out, plain = perception
    g = H.load('iou_b4.npz')
    present = model.receptive_field - 1

    def iou(c):
        return float(c[0]) / max(1.0, float(np.sum(c)))

    def unpack(key, shape):
        return torch.from_numpy(np.unpackbits(g[key], axis=1).astype(np.int64)).reshape(shape)

    for key in H.IOU_HEADS:
        pred = out[key].float().argmax(dim=2)
        disagreement = (pred.cpu() != unpack(f'pred/{key}', tuple(pred.shape))).float().mean().item()
        print(f'[inference] {key}: arg-max disagreement with the reference {disagreement:.2e} (bound 1e-3)')
        for lname, tgt, bound in (('synthetic', batch[key][:, :, 0], 1e-3), ('pseudo', unpack(f'pseudo/{key}', tuple(pred.shape)), 2e-2)):
            for fname, sl in (('present', slice(present, None)), ('all', slice(None))):
                metric = IntersectionOverUnion(2).cuda()
                metric(pred[:, sl].unsqueeze(2), tgt[:, sl].unsqueeze(2).cuda())
                got, want = metric.compute()[1].item(), iou(g[f'counts/{key}/{lname}/{fname}'])
                print(f'[inference] {key}/{lname}/{fname}: IoU {got:.6f}, reference {want:.6f}, diff {abs(got - want):.2e} (bound {bound})')
                assert abs(got - want) <= bound, (key, lname, fname, got, want)
        assert disagreement <= 1e-3, (key, disagreement)


def _check_refresh(model, batch, engine, out):
    """load_state_dict of perturbed weights and running statistics: the engine is stale until ``refresh()`` and equal to the
    plain forward after it.  The plain forward on the changed weights runs LAST: an eager forward rewrites the bf16 shadows by
    itself (their version check), so run before ``refresh()`` it would hide a ``refresh()`` that forgot them."""
    original = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator(device='cuda').manual_seed(5)
    changed = {}
    for k, v in original.items():
        if not v.is_floating_point():
            changed[k] = v
        elif k.endswith('running_var'):
            changed[k] = v * (1.0 + 0.2 * torch.rand(v.shape, generator=g, device=v.device))
        else:
            changed[k] = v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g, device=v.device)
    try:
        model.load_state_dict(changed)
        stale = engine(*_inputs(batch), clone=True)            # no eager forward yet: nothing has refreshed anything
        engine.refresh()
        fresh = engine(*_inputs(batch), clone=True)            # still none: refresh() alone brought the engine up to date
        want = _plain(model, batch)
        stale_bad = _mismatches(stale, want)
        print('[inference] without refresh(): entries that differ from the plain forward', sorted(stale_bad))
        assert stale_bad, 'the engine followed a weight change without refresh(): it does not read the shadows / the arena'
        bad = _mismatches(fresh, want)
        print('[inference] after refresh(): mismatching elements', bad)
        assert not bad, bad
        assert _mismatches(fresh, out), 'perturbed weights gave the original outputs'
        # the eager forward above went through every weight cache with the new values: whatever it replaced there, the graph
        # must not have been reading it
        bad = _mismatches(engine(*_inputs(batch), clone=True), want)
        assert not bad, ('after an eager forward on the new weights', bad)
    finally:
        model.load_state_dict(original)
        engine.refresh()
    assert not _mismatches(engine(*_inputs(batch), clone=True), out)
    assert not _mismatches(_plain(model, batch), out)
    assert not _mismatches(engine(*_inputs(batch), clone=True), out)


def test_refresh_after_load_state_dict(perception):
    model, batch, engine, out, plain = perception
    _check_refresh(model, batch, engine, out)


def test_error_paths(perception):
    from stp3_amd._lib import Stp3HipError
    from stp3_amd.inference import InferenceEngine
    from stp3_amd.models.stp3 import STP3
    model, batch, engine, out, plain = perception
    small = synthetic.make_batch(batch=2, seq=3, seed=7)
    with pytest.raises(Stp3HipError, match='shape'):
        engine(*_inputs(small))
    model.train()
    try:
        with pytest.raises(Stp3HipError, match='training'):
            engine(*_inputs(batch))
        with pytest.raises(Stp3HipError, match='training'):
            InferenceEngine(model, batch)
    finally:
        model.eval()
    with pytest.raises(Stp3HipError, match='CPU'):
        InferenceEngine(STP3(perception_cfg()).eval(), small)
    assert not _mismatches(engine(*_inputs(batch), clone=True), out)       # the engine is unharmed


def test_perception_b1_bit_equal(perception):
    from stp3_amd.inference import InferenceEngine
    model = perception[0]
    batch = synthetic.make_batch(batch=1, seq=3, seed=3)
    want = _plain(model, batch)
    example = batch['image'].cuda()
    kept = example.clone()
    engine = InferenceEngine(model, (example,) + tuple(batch[k] for k in POSES), autocast_dtype=torch.bfloat16)
    bad = _mismatches(engine(*_inputs(batch), clone=True), want)
    print('[inference] Perception B=1: mismatching elements', bad)
    assert not bad, bad
    # the static input buffer is the engine's own: a later call does not write the caller's example tensor
    other = synthetic.make_batch(batch=1, seq=3, seed=4)
    engine(*_inputs(other))
    assert engine.image.data_ptr() != example.data_ptr() and torch.equal(example, kept)
    assert not torch.equal(engine.image, kept)


def test_float32_engine_bit_equal(perception):
    """No autocast: the plain float32 operators are captured unfused."""
    from stp3_amd.inference import InferenceEngine
    model = perception[0]
    batch = synthetic.make_batch(batch=1, seq=3, seed=3)
    want = _plain(model, batch, dtype=None)
    engine = InferenceEngine(model, batch, autocast_dtype=None)
    assert engine.coefs is None
    got = engine(*_inputs(batch), clone=True)
    assert got['segmentation'].dtype == torch.float32
    bad = _mismatches(got, want)
    print('[inference] float32 engine: mismatching elements', bad)
    assert not bad, bad


@pytest.fixture(scope='module')
def prediction():
    """(model, batch, engine, engine outputs, plain outputs), Prediction.yml-shaped (N_FUTURE_FRAMES = 4, GAUSSIAN present
    distribution; eval mode samples with zero noise) at the size tests/test_prediction_gpu.py uses."""
    from stp3_amd.inference import InferenceEngine
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    from tests.test_prediction_cpu import PREDICTION
    model = to_channels_last(H.fill_deterministic(STP3(perception_cfg(**PREDICTION))).eval().cuda())
    batch = synthetic.make_batch(batch=1, seq=7, seed=3, instance=True)
    plain = _plain(model, batch)
    engine = InferenceEngine(model, batch, autocast_dtype=torch.bfloat16)
    out = engine(*_inputs(batch), clone=True)
    return model, batch, engine, out, plain


def test_prediction_bit_equal(prediction):
    model, batch, engine, got, want = prediction
    assert got['segmentation'].shape[:2] == (1, 7)
    bad = _mismatches(got, want)
    print('[inference] Prediction B=1: entries', sorted(k for k, v in got.items() if v is not None), 'mismatching elements', bad)
    assert not bad, bad
    assert engine.gates.entries, 'the GRU cells of the prediction stage did not take the engine\'s gate weights'


def test_prediction_refresh_after_load_state_dict(prediction):
    """The GRU cells read MERGED gate weights and biases, cut from the parameters' shadows: ``refresh()`` must rewrite those
    too, in place (the graph holds their addresses)."""
    model, batch, engine, out, plain = prediction
    merged = [(wb.data_ptr(), wb.clone(), bias.data_ptr(), bias.clone()) for _, _, wb, bias in engine.gates.entries.values()]
    _check_refresh(model, batch, engine, out)
    for (pw, w0, pb, b0), (_, _, wb, bias) in zip(merged, engine.gates.entries.values()):
        assert (wb.data_ptr(), bias.data_ptr()) == (pw, pb)
        assert torch.equal(wb, w0) and torch.equal(bias, b0)           # (restored with the original weights)
