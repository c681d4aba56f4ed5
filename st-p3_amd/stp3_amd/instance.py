"""Vehicle instance post-processing (``stp3/utils/instance.py:80-330``): centerness / offset / flow heads -> temporally
consistent instance ids, with the reference's public surface -- ``find_instance_centers``, ``group_pixels``,
``get_instance_segmentation_and_centers``, ``update_instance_ids``, ``make_instance_seg_consecutive``,
``make_instance_id_temporally_consistent``, ``predict_instance_segmentation_and_trajectories``.

GPU tensors go through two launches of csrc/stp3_instance.hip (``stp3_instance_segment`` for all B * S frames,
``stp3_instance_track`` for all B samples with the loop over time inside) plus dtype conversions, with no host
synchronisation; CPU tensors take the torch path of this file, which the CPU tests pin on the reference's recorded results
and which states the rules both follow:

* a centre: value ``> conf_threshold`` (and ``> 0``) that equals the maximum of its 3x3 neighbourhood (all tied pixels of
  a plateau; a NaN in the neighbourhood disqualifies), numbered in row-major order, cut to the first 100;
* a pixel's instance: the centre ``k`` with the lowest float32 ``sqrt(dr * dr + dc * dc)`` to ``pixel + offset`` -- the lowest
  ``k`` on equal values -- times the foreground mask, then ranked among the distinct values of the masked map (a frame
  without background has no value 0: its lowest id becomes 0, as in the reference);
* tracking, per sample and step: rows = the ids of the consistent frame ``t`` in ascending order with the mean of
  ``(row, col) + flow[t]`` over their pixels, columns = ids ``1..n`` of the raw frame ``t + 1`` with their pixel means,
  float32 Euclidean distances, minimum-cost assignment (``lsap``: shortest augmenting paths, the smaller side first),
  matches closer than ``matching_threshold`` kept.  Means are exact: coordinates are summed as integers, the flow in
  fixed point (2^-20 pixel, round to nearest even), divided in float64 and rounded once to float32;
* **fresh ids** -- every unmatched id of ``t + 1`` gets ``++largest_instance_id`` in ASCENDING order of its old id.  The
  reference iterates a Python ``set`` of numpy integers there (instance.py:257-264: hash-table order, not ascending in about
  one step in ten), so its result equals this one up to a renaming of ids created after frame 0 at the same step --
  invisible downstream: ``PanopticMetric`` compares ids for equality within a sample and ``matched_centers`` is keyed by
  frame-0 ids.

Inputs the tracker refuses (the reference fails on them too, with a NaN cost matrix or a KeyError): ids of a raw frame that
are not ``0..n`` with every value present, a frame without a background pixel, ids above 100, non-finite or |flow| >= 32768.
The torch path raises ``ValueError``; the kernel sets a word of its error output, treats the value as background / zero and
runs to its end (``check=True``, or ``compute_matched_centers=True`` which synchronises anyway, reads the word and raises).
"""
import numpy as np
import torch
import torch.nn.functional as F

MAX_CENTERS = 100                       # max_n_instance_centers of the reference; the kernels' table size
MAX_SIDE, MAX_PIXELS = 1024, 1 << 24    # stp3_instance_segment / _track: H, W <= 1024 and H * W < 2^24 (else the torch path)
FLOW_SCALE = float(1 << 20)             # fixed point of the flow sums
FLOW_LIMIT = 32768.0
ERRORS = ('the assignment hit its iteration bound', 'raw instance ids are not 0..n <= 100 with every id present',
          'a frame has no background pixel', 'non-finite or huge flow on an instance pixel')      # the words of `err`


class InstanceError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------------
# the reference's single-frame functions
# ------------------------------------------------------------------------------------------------------------------
def _center_mask(center_prediction, conf_threshold=0.1, nms_kernel_size=3):
    """(N, H, W) bool: the candidate centres of N frames at once (instance.py:82-91)."""
    x = F.threshold(center_prediction.float(), threshold=conf_threshold, value=-1.0)
    pad = (nms_kernel_size - 1) // 2
    pooled = F.max_pool2d(x.unsqueeze(1), kernel_size=nms_kernel_size, stride=1, padding=pad).squeeze(1)
    return (x == pooled) & (x > 0)


def find_instance_centers(center_prediction, conf_threshold=0.1, nms_kernel_size=3):
    assert len(center_prediction.shape) == 3
    return torch.nonzero(_center_mask(center_prediction, conf_threshold, nms_kernel_size))[:, 1:]


def _nearest_center(centers, offset):
    """(H, W) int64: index of the nearest centre ((K, 2) integers, K >= 1) to pixel + offset ((2, H, W) float32)."""
    h, w = offset.shape[-2:]
    rows = torch.arange(h, dtype=torch.float32, device=offset.device).view(h, 1) + offset[0]
    cols = torch.arange(w, dtype=torch.float32, device=offset.device).view(1, w) + offset[1]
    c = centers.to(torch.float32)
    dr = c[:, 0].view(-1, 1, 1) - rows
    dc = c[:, 1].view(-1, 1, 1) - cols
    return torch.argmin(torch.sqrt(dr * dr + dc * dc), dim=0)


def group_pixels(centers, offset_predictions):
    return (_nearest_center(centers, offset_predictions.float().reshape(2, *offset_predictions.shape[-2:])) + 1).unsqueeze(0)


def update_instance_ids(instance_seg, old_ids, new_ids):
    indices = torch.arange(int(old_ids.max()) + 1, device=instance_seg.device)
    indices[old_ids.long()] = new_ids.long().to(indices.device)
    return indices[instance_seg].long()


def make_instance_seg_consecutive(instance_seg):
    unique_ids = torch.unique(instance_seg)
    return update_instance_ids(instance_seg, unique_ids, torch.arange(len(unique_ids), device=instance_seg.device))


def get_instance_segmentation_and_centers(center_predictions, offset_predictions, foreground_mask, conf_threshold=0.1,
                                          nms_kernel_size=3, max_n_instance_centers=MAX_CENTERS):
    h, w = center_predictions.shape[-2:]
    seg, centers, counts = segment_frames(center_predictions.reshape(1, h, w), offset_predictions.reshape(1, 2, h, w),
                                          foreground_mask.reshape(1, h, w), conf_threshold, nms_kernel_size,
                                          max_n_instance_centers)
    return seg.long(), centers[0, :int(counts[0])].long()       # (a data-dependent shape: one synchronisation on the GPU)


# ------------------------------------------------------------------------------------------------------------------
# all frames at once
# ------------------------------------------------------------------------------------------------------------------
def _kernel_ok(t, h, w):
    return t.is_cuda and h <= MAX_SIDE and w <= MAX_SIDE and h * w < MAX_PIXELS


def segment_frames(center, offset, foreground, conf_threshold=0.1, nms_kernel_size=3, max_n_instance_centers=MAX_CENTERS):
    """N frames: centerness (N, H, W), offset (N, 2, H, W), foreground (N, H, W) bool / uint8 -> instance ids (N, H, W)
    int32, centres (N, 100, 2) int32 (row, column; zero beyond the count), counts (N,) int32."""
    n, h, w = center.shape
    assert offset.shape == (n, 2, h, w) and foreground.shape == (n, h, w)
    if _kernel_ok(center, h, w) and nms_kernel_size == 3 and max_n_instance_centers == MAX_CENTERS and n > 0:
        return _segment_frames_kernel(center, offset, foreground, conf_threshold)
    return segment_frames_reference(center, offset, foreground, conf_threshold, nms_kernel_size, max_n_instance_centers)


def segment_frames_reference(center, offset, foreground, conf_threshold=0.1, nms_kernel_size=3,
                             max_n_instance_centers=MAX_CENTERS):
    """The torch path of ``segment_frames``: candidates and the renumbering for all frames together; the distance table of a
    frame (K x H x W float32, 16 MB at 100 centres and 200 x 200) is built frame by frame to bound the memory."""
    n, h, w = center.shape
    dev = center.device
    center, offset = center.detach().float(), offset.detach().float()
    mask = _center_mask(center, conf_threshold, nms_kernel_size)
    order = torch.cumsum(mask.view(n, -1), dim=1)                                  # 1-based rank in row-major order
    keep = mask.view(n, -1) & (order <= max_n_instance_centers)
    counts = keep.sum(dim=1).to(torch.int32)
    centers = torch.zeros(n, max_n_instance_centers, 2, dtype=torch.int32, device=dev)
    f, p = torch.nonzero(keep, as_tuple=True)
    k = order[f, p] - 1
    centers[f, k, 0] = torch.div(p, w, rounding_mode='floor').to(torch.int32)
    centers[f, k, 1] = (p % w).to(torch.int32)
    seg = torch.zeros(n, h, w, dtype=torch.int64, device=dev)
    fg = foreground.reshape(n, h, w) != 0
    for i in range(n):
        c = int(counts[i])
        if c:
            seg[i] = (_nearest_center(centers[i, :c], offset[i]) + 1) * fg[i]
    # make_instance_seg_consecutive per frame: rank among the distinct values of the masked map
    present = torch.zeros(n, max_n_instance_centers + 1, dtype=torch.bool, device=dev)
    present.scatter_(1, seg.view(n, -1), True)
    rank = torch.cumsum(present, dim=1) - 1
    seg = torch.gather(rank, 1, seg.view(n, -1)).view(n, h, w)
    return seg.to(torch.int32), centers, counts


def _segment_frames_kernel(center, offset, foreground, conf_threshold):
    from . import _lib, ops
    n, h, w = center.shape
    center = center.detach().float().contiguous()
    offset = offset.detach().float().contiguous()
    fg = foreground.detach().to(torch.uint8).contiguous()
    seg = torch.empty(n, h, w, dtype=torch.int32, device=center.device)
    centers = torch.empty(n, MAX_CENTERS, 2, dtype=torch.int32, device=center.device)
    counts = torch.empty(n, dtype=torch.int32, device=center.device)
    _lib.check(_lib.lib().stp3_instance_segment(n, h, w, float(conf_threshold), ops._ptr(center), ops._ptr(offset), ops._ptr(fg),
                                                ops._ptr(seg), ops._ptr(centers), ops._ptr(counts), ops._stream()),
               'stp3_instance_segment')
    return seg, centers, counts


# ------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------
def lsap(cost):
    """Minimum-cost assignment of a rectangular matrix, every row or every column (the smaller side) assigned: (rows, cols)
    in ascending row order, like ``scipy.optimize.linear_sum_assignment``.  Shortest augmenting paths with dual variables
    (Jonker-Volgenant as restated by Crouse, "On implementing 2D rectangular assignment algorithms", 2016 -- the method
    scipy uses), float64 arithmetic, one augmentation per row of the smaller side; among equally short paths an unassigned
    column is preferred, the one scanned last, else the one scanned first, the scan going over the not yet visited
    columns kept in a list from which a visited one is removed by moving the last into its place.  The kernel
    (csrc/stp3_instance.hip, ``assign``) restates exactly this, so that both give the same pairs even between equal optima."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError('lsap: a matrix is expected')
    if not np.isfinite(cost).all():
        raise ValueError('lsap: non-finite cost')
    transposed = cost.shape[1] < cost.shape[0]
    if transposed:
        cost = cost.T
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        spc = np.full(nc, np.inf)
        path = np.full(nc, -1)
        remaining = np.arange(nc - 1, -1, -1)
        visited_rows, visited_cols = [], []
        min_val, i, sink = 0.0, cur, -1
        for _ in range(nc):                                     # every turn visits one more column: at most nc
            visited_rows.append(i)
            r = min_val + cost[i, remaining] - u[i] - v[remaining]
            better = r < spc[remaining]
            spc[remaining[better]] = r[better]
            path[remaining[better]] = i
            vals = spc[remaining]
            min_val = vals.min()
            at = np.nonzero(vals == min_val)[0]
            free = at[row4col[remaining[at]] < 0]
            index = free[-1] if len(free) else at[0]
            j = remaining[index]
            visited_cols.append(j)
            remaining[index] = remaining[-1]
            remaining = remaining[:-1]
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        if sink < 0:
            raise RuntimeError('lsap: no augmenting path within its bound')
        u[cur] += min_val
        for i in visited_rows:
            if i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in visited_cols:
            v[j] -= min_val - spc[j]
        j = sink
        for _ in range(nr + 1):
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows = np.arange(nr)
    if transposed:
        order = np.argsort(col4row)
        return col4row[order], rows[order]
    return rows, col4row.copy()


# ------------------------------------------------------------------------------------------------------------------
# tracking
# ------------------------------------------------------------------------------------------------------------------
def _frame_stats(ids, flow, n_ids):
    """Per id 0..n_ids-1 of an (H, W) id map: pixel count, integer row / column sums, fixed-point flow sums (int64)."""
    h, w = ids.shape
    flat = ids.reshape(-1)
    rows = torch.arange(h, dtype=torch.int64).view(h, 1).expand(h, w).reshape(-1)
    cols = torch.arange(w, dtype=torch.int64).view(1, w).expand(h, w).reshape(-1)
    zero = torch.zeros(n_ids, dtype=torch.int64)
    out = [torch.bincount(flat, minlength=n_ids), zero.index_add(0, flat, rows), zero.index_add(0, flat, cols)]
    if flow is not None:
        if not bool((flow.abs() < FLOW_LIMIT)[:, ids > 0].all()):
            raise InstanceError(ERRORS[3])
        fx = torch.round(torch.where(ids > 0, flow, torch.zeros_like(flow)).double() * FLOW_SCALE).to(torch.int64).reshape(2, -1)
        out += [zero.index_add(0, flat, fx[0]), zero.index_add(0, flat, fx[1])]
    return out


def _means(cnt, sr, sc, fr=None, fc=None):
    """float32 (n, 2): (integer sum + fixed-point sum * 2^-20) / count in float64, rounded once."""
    r, c = sr.double(), sc.double()
    if fr is not None:
        r, c = r + fr.double() * (1.0 / FLOW_SCALE), c + fc.double() * (1.0 / FLOW_SCALE)
    return torch.stack([r / cnt.double(), c / cnt.double()], dim=1).float()


def step_distances(cur, nxt, flow_t, ids_t, n):
    """The cost matrix of one step, float32 numpy (len(ids_t), n): rows = the ids ``ids_t`` of the consistent frame ``cur`` warped
    by ``flow_t`` ((2, H, W) or None), columns = ids 1..n of the raw frame ``nxt`` (instance.py:201-239)."""
    cnt, sr, sc, fr, fc = _frame_stats(cur, flow_t if flow_t is not None else torch.zeros(2, *cur.shape), int(ids_t[-1]) + 1)
    warped = _means(cnt[ids_t], sr[ids_t], sc[ids_t], fr[ids_t], fc[ids_t])
    cnt, sr, sc = _frame_stats(nxt, None, n + 1)
    if int(cnt[1:].min()) == 0 or n > MAX_CENTERS:
        raise InstanceError(ERRORS[1])
    actual = _means(cnt[1:], sr[1:], sc[1:])
    d = actual.unsqueeze(0) - warped.unsqueeze(1)
    return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).numpy()


def _track_sample(raw, flow, matching_threshold):
    """One sample: raw (S, H, W) int64 on the CPU, flow (S, 2, H, W) float32 or None -> consistent ids (S, H, W) int64."""
    s = raw.shape[0]
    thr = np.float32(matching_threshold)
    out = [raw[0]]
    largest = int(raw[0].max())
    for t in range(s - 1):
        cur, nxt = out[-1], raw[t + 1]
        n = int(nxt.max())
        ids_t = torch.unique(cur)
        if int(ids_t[0]) != 0 or int(nxt.min()) != 0:
            raise InstanceError(ERRORS[2])
        ids_t = ids_t[1:]
        if len(ids_t) == 0 or n == 0:                           # instance.py:211-214, 228-231: the raw frame is taken over
            out.append(nxt)
            continue
        dist = step_distances(cur, nxt, flow[t] if flow is not None else None, ids_t, n)
        ri, ci = lsap(dist)
        good = dist[ri, ci] < thr
        new_ids = np.zeros(n + 1, dtype=np.int64)
        new_ids[ci[good] + 1] = ids_t.numpy()[ri[good]]
        fresh = np.nonzero(new_ids[1:] == 0)[0] + 1             # ascending old id: this project's rule (see the module text)
        new_ids[fresh] = largest + 1 + np.arange(len(fresh))
        largest += len(fresh)
        out.append(torch.from_numpy(new_ids)[nxt])
    return torch.stack(out)


def track_frames_reference(raw, flow, matching_threshold=3.0):
    """The torch path of ``track_frames``: raw (B, S, H, W) ids, flow (B, S, 2, H, W) or None -> consistent ids, int64."""
    raw = raw.detach().long().cpu()
    if flow is not None:
        flow = flow.detach().float().cpu()
    return torch.stack([_track_sample(raw[b], flow[b] if flow is not None else None, matching_threshold)
                        for b in range(raw.shape[0])])


def track_frames(raw, flow, matching_threshold=3.0, check=False):
    """raw (B, S, H, W) integer ids of ``segment_frames`` (per frame 0..n, every value present), flow (B, S, 2, H, W) float32
    or None (zero flow) -> (temporally consistent ids (B, S, H, W), error word): int32 ids and a four-element int32 device
    tensor from the kernel (GPU tensors, one launch, no synchronisation unless ``check``), int64 ids and None from the
    torch path (which raises by itself)."""
    b, s, h, w = raw.shape
    if not (_kernel_ok(raw, h, w) and b > 0 and s > 0):
        return track_frames_reference(raw, flow, matching_threshold).to(raw.device), None
    from . import _lib, ops
    raw = raw.detach().to(torch.int32).contiguous()
    if flow is not None:
        assert flow.shape == (b, s, 2, h, w)
        flow = flow.detach().float().contiguous()
    out = torch.empty_like(raw)
    err = torch.zeros(4, dtype=torch.int32, device=raw.device)
    _lib.check(_lib.lib().stp3_instance_track(b, s, h, w, float(matching_threshold), ops._ptr(raw),
                                              ops._ptr(flow) if flow is not None else None, ops._ptr(out), ops._ptr(err),
                                              ops._stream()), 'stp3_instance_track')
    if check:
        raise_on_error(err)
    return out, err


def raise_on_error(err):
    words = err.tolist()                           # (synchronises)
    if any(words):
        raise InstanceError('stp3_instance_track: ' + '; '.join(e for e, w in zip(ERRORS, words) if w))


def make_instance_id_temporally_consistent(pred_inst, future_flow, matching_threshold=3.0):
    """instance.py:173-269 for any batch size: pred_inst (B, S, H, W), future_flow (B, S, 2, H, W) -> (B, S, H, W) int64."""
    return track_frames(pred_inst, future_flow, matching_threshold)[0].long()


def matched_centers_of(consistent):
    """instance.py:308-328: {frame-0 id: float32 array (frames in which the id has pixels, 2) as (column, row)} of sample 0."""
    seq = consistent[0].detach().long()
    s, h, w = seq.shape
    n0 = int(seq[0].max())                         # (synchronises: the result is host data)
    if n0 == 0:
        return {}
    ids = torch.where(seq <= n0, seq, torch.zeros_like(seq))
    key = (ids + (n0 + 1) * torch.arange(s, device=seq.device).view(s, 1, 1)).reshape(-1)
    rows = torch.arange(h, dtype=torch.float64, device=seq.device).view(1, h, 1).expand(s, h, w).reshape(-1)
    cols = torch.arange(w, dtype=torch.float64, device=seq.device).view(1, 1, w).expand(s, h, w).reshape(-1)
    m = s * (n0 + 1)
    cnt = torch.bincount(key, minlength=m).double()
    table = torch.stack([cnt, torch.bincount(key, weights=rows, minlength=m), torch.bincount(key, weights=cols, minlength=m)])
    cnt, sr, sc = table.view(3, s, n0 + 1).cpu().numpy()
    present0 = cnt[0] > 0
    out = {}
    for i in range(1, n0 + 1):
        if not present0[i]:
            continue
        t = np.nonzero(cnt[:, i] > 0)[0]
        out[np.int64(i)] = np.stack([sc[t, i] / cnt[t, i], sr[t, i] / cnt[t, i]], axis=1).astype(np.float32)
    return out


def predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False, make_consistent=True, vehicles_id=1,
                                                   check=False):
    """instance.py:272-330.  ``output``: 'segmentation' (B, S, C, H, W) logits, 'instance_center' (B, S, 1, H, W),
    'instance_offset' (B, S, 2, H, W), 'instance_flow' (B, S, 2, H, W) or None (zero flow; the dictionary is not written to).
    Returns the consistent instance ids (B, S, H, W) int64, and with ``compute_matched_centers`` (B == 1) the dictionary of
    ``matched_centers_of``.  ``check``: read the tracker's error word (one synchronisation) and raise on it."""
    seg_logits = output['segmentation'].detach()
    b, s = seg_logits.shape[:2]
    h, w = seg_logits.shape[-2:]
    foreground = torch.argmax(seg_logits, dim=2) == vehicles_id
    raw, _, _ = segment_frames(output['instance_center'].detach().reshape(b * s, h, w),
                               output['instance_offset'].detach().reshape(b * s, 2, h, w), foreground.reshape(b * s, h, w))
    raw = raw.view(b, s, h, w)
    if make_consistent:
        flow = output.get('instance_flow')
        tracked, err = track_frames(raw, flow)
        consistent = tracked.long()
        if err is not None and (check or compute_matched_centers):
            raise_on_error(err)
    else:
        consistent = raw.long()
    if compute_matched_centers:
        assert b == 1
        return consistent, matched_centers_of(consistent)
    return consistent
